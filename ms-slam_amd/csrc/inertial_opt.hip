// Optimizer::InertialOptimization (src/Optimizer.cc:3050-3227, :3230-3384, :3386-3491) after its gathering loops: the whole
// optimize(its) in ONE launch, in double like g2o with the preintegration's bias correction in float like the reference.  The
// arithmetic is inertial_device.h, the same text a host compiler reads; this file is the executor that spreads it over a workgroup,
// and the entry.
//
// One workgroup of 256 threads owns the call, as in pose_opt.hip and sim3_opt.hip: the typical call (InitializeIMU at 10 to about
// 100 KeyFrames) is a few hundred dependent passes over a few dozen edges, which a host-driven loop would pay two read-backs per
// iteration for.  One wavefront per SIMD leaves the double-precision Jacobians the whole register file.
//
// A pass: thread t linearises the edges t, t + 256, ... into the workspace in global memory (135 doubles an edge); a second step adds
// each velocity's at most two contributions, the previous edge first; the border's sums go through the fixed-order tree (per thread
// ascending, xor butterfly 32..1 in a wavefront, the four wavefronts in ascending order through a double-buffered LDS block).  The
// solve is a block cyclic reduction of the tridiagonal part carrying the border's columns, one thread per surviving block row per
// level, then the border's Schur complement factored by every thread redundantly, then the back-substitution.  No atomics: two
// runs give the same bits.  Every trip count comes from reduced values that all threads hold with equal bits, so every thread
// reaches every barrier.  All per-row state is in global memory, which L2 holds at the capacity of 4096 KeyFrames.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/msorb.h"
#include "hip_host.h"
#include "inertial_device.h"
#include "inertial_plan.h"

namespace msorb {
hipError_t small_copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s);   // orb_kernels.hip
}
using msorb::set_last_error;
using msorb::ThreadScratch;
using msorb::up16;
using namespace msorb::inertial;

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64, kCapacity = 4096;
constexpr int kMaxIterations = 10000;   // the callers ask for 200 and 10; one launch runs them all, so the count is bounded

static_assert(sizeof(msorb_inertial_keyframe) == 128 && sizeof(msorb_inertial_edge) == 928 && sizeof(msorb_inertial_problem) == 184 &&
                  sizeof(msorb_inertial_result) == 160,
              "the records of include/msorb.h as the Python mirror lays them out");

struct InertialArgs {
    Work K;
    const msorb_inertial_problem* problem;
    msorb_inertial_result* result;
};

struct BlockExec {
    double* const lds;   // 2 blocks of kWaves * kSumMax
    int buf = 0;
    __device__ explicit BlockExec(double* l) : lds(l) {}
    __device__ inline int tid() const { return threadIdx.x; }
    __device__ inline int stride() const { return kThreads; }
    __device__ inline void barrier() { __syncthreads(); }

    // block_sum of pose_opt.hip: every thread returns with the same bits; the two LDS blocks alternate, so the one barrier also
    // protects the block of the reduction before the last
    __device__ inline void sum(double* v, int n) {
        double* l = lds + (buf ^= 1) * kWaves * kSumMax;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
            for (int i = 0; i < kSumMax; i++)
                if (i < n) v[i] += msorb::se3::shfl_xor_f64(v[i], off);
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0)
#pragma unroll
            for (int i = 0; i < kSumMax; i++)
                if (i < n) l[wave * kSumMax + i] = v[i];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kSumMax; i++)
            if (i < n) {
                double s = l[i];
                for (int w = 1; w < kWaves; w++) s += l[w * kSumMax + i];
                v[i] = s;
            }
    }

    __device__ inline double max1(double v) {
        double* l = lds + (buf ^= 1) * kWaves * kSumMax;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v = fmax(v, msorb::se3::shfl_xor_f64(v, off));
        if ((threadIdx.x & 63) == 0) l[threadIdx.x >> 6] = v;
        __syncthreads();
        double s = l[0];
        for (int w = 1; w < kWaves; w++) s = fmax(s, l[w]);
        return s;
    }
};

__global__ __launch_bounds__(kThreads) void inertial_opt_kernel(const InertialArgs A) {
    __shared__ double lds[2 * kWaves * kSumMax];
    BlockExec ex(lds);
    const msorb_inertial_problem P = *A.problem;
    optimize(ex, A.K, P, *A.result);
}

// Staging.  Up: [problem | kfs | edges | row_kf | e_prev | e_next]; down: [result | v | chi2]; the rest stays on the device.
struct Staged {
    size_t o_prob, o_kf, o_edge, o_row, o_ep, o_en, in_bytes, o_res, o_v, o_chi2, out_end, o_W, o_D, o_L, o_U, o_R, o_R0, o_x, bytes;
    Staged(size_t nk, size_t ne, size_t nr) {
        o_prob = 0;
        o_kf = up16(sizeof(msorb_inertial_problem));
        o_edge = o_kf + up16(nk * sizeof(msorb_inertial_keyframe));
        o_row = o_edge + up16(ne * sizeof(msorb_inertial_edge));
        o_ep = o_row + up16(nr * 4);
        o_en = o_ep + up16(nr * 4);
        in_bytes = o_en + up16(nr * 4);
        o_res = in_bytes;
        o_v = o_res + up16(sizeof(msorb_inertial_result));
        o_chi2 = o_v + up16(nk * 48);          // both copies of Work::v; the callers read the first
        out_end = o_chi2 + up16(ne * 8);
        o_W = out_end;
        o_D = o_W + up16(ne * kEdgeW * 8);
        o_L = o_D + up16(nr * 72);
        o_U = o_L + up16(nr * 72);
        o_R = o_U + up16(nr * 72);
        o_R0 = o_R + up16(nr * 24 * kRhs);
        o_x = o_R0 + up16(nr * 24 * kRhs);
        bytes = o_x + up16(nr * 24);
    }
};

bool finite_all(const double* p, int n) {
    for (int i = 0; i < n; i++)
        if (!std::isfinite(p[i])) return false;
    return true;
}
bool finite_all(const float* p, int n) {
    for (int i = 0; i < n; i++)
        if (!std::isfinite(p[i])) return false;
    return true;
}

}  // namespace

extern "C" int msorb_inertial_optimization_capacity(void) { return kCapacity; }

extern "C" int msorb_inertial_optimization(int device, const msorb_inertial_problem* p, int n_kf, const msorb_inertial_keyframe* kfs,
                                           int n_edges, const msorb_inertial_edge* edges, double* v_out, double* edge_chi2,
                                           msorb_inertial_result* r, float* elapsed_ms) {
    if (!p || !r || n_kf < 0 || n_edges < 0 || (n_kf > 0 && (!kfs || !v_out)) || (n_edges > 0 && !edges)) {
        set_last_error("inertial_optimization: a null required pointer or a negative count");
        return MSORB_E_INVALID;
    }
    if (p->iterations < 0 || p->iterations > kMaxIterations || (p->algorithm != 0 && p->algorithm != 1)) {
        set_last_error("inertial_optimization: iterations below 0 or above 10000, or an unknown algorithm");
        return MSORB_E_INVALID;
    }
    if (n_kf > kCapacity) {
        set_last_error("inertial_optimization: more KeyFrames than msorb_inertial_optimization_capacity()");
        return MSORB_E_CAPACITY;
    }
    if (!finite_all(p->Rwg, 9) || !finite_all(&p->scale, 1) || !finite_all(p->bg, 3) || !finite_all(p->ba, 3) ||
        !finite_all(&p->prior_g, 1) || !finite_all(&p->prior_a, 1)) {
        set_last_error("inertial_optimization: a non-finite value in the problem");
        return MSORB_E_INVALID;
    }
    for (int k = 0; k < n_kf; k++)
        if (!finite_all(kfs[k].Rwb, 15)) {   // Rwb, twb, v are contiguous doubles
            set_last_error("inertial_optimization: a non-finite value in a KeyFrame");
            return MSORB_E_INVALID;
        }
    std::vector<int> prev(n_edges), cur(n_edges);
    for (int e = 0; e < n_edges; e++) {
        const msorb_inertial_edge& E = edges[e];
        if (E.kf_prev < 0 || E.kf_prev >= n_kf || E.kf_cur < 0 || E.kf_cur >= n_kf || E.kf_prev == E.kf_cur) {
            set_last_error("inertial_optimization: an edge names a KeyFrame out of range, or one KeyFrame twice");
            return MSORB_E_INVALID;
        }
        if (!kfs[E.kf_prev].has_velocity_vertex || !kfs[E.kf_cur].has_velocity_vertex) {
            set_last_error("inertial_optimization: an edge on a KeyFrame without velocity vertex");
            return MSORB_E_INVALID;
        }
        if (!finite_all(E.dR, 67) || !finite_all(E.info, 81)) {   // dR .. dT are contiguous floats
            set_last_error("inertial_optimization: a non-finite value in an edge");
            return MSORB_E_INVALID;
        }
        prev[e] = E.kf_prev;
        cur[e] = E.kf_cur;
    }
    Plan plan;
    if (make_plan(n_kf, n_edges, prev.data(), cur.data(), plan) != kPlanOk) {
        set_last_error("inertial_optimization: the edges do not form chains (a KeyFrame with two edges on one side, or a cycle)");
        return MSORB_E_CAPACITY;
    }
    if (int rc = msorb::require_device(device)) return rc;
    const size_t nk = (size_t)n_kf, ne = (size_t)n_edges, nr = plan.row_kf.size();
    const Staged L(nk, ne, nr);
    static thread_local ThreadScratch scr(true, 2);
    if (int rc = scr.acquire(device, L.bytes, L.out_end)) return rc;
    uint8_t *const h = scr.h.p, *const d = scr.d.p;
    std::memcpy(h + L.o_prob, p, sizeof(*p));
    if (nk) std::memcpy(h + L.o_kf, kfs, nk * sizeof(*kfs));
    if (ne) std::memcpy(h + L.o_edge, edges, ne * sizeof(*edges));
    if (nr) {
        std::memcpy(h + L.o_row, plan.row_kf.data(), nr * 4);
        std::memcpy(h + L.o_ep, plan.e_prev.data(), nr * 4);
        std::memcpy(h + L.o_en, plan.e_next.data(), nr * 4);
    }
    InertialArgs A{};
    A.K.n_kf = n_kf; A.K.n_edges = n_edges; A.K.n_rows = (int)nr;
    A.K.kf = reinterpret_cast<const msorb_inertial_keyframe*>(d + L.o_kf);
    A.K.edge = reinterpret_cast<const msorb_inertial_edge*>(d + L.o_edge);
    A.K.row_kf = reinterpret_cast<const int*>(d + L.o_row);
    A.K.e_prev = reinterpret_cast<const int*>(d + L.o_ep);
    A.K.e_next = reinterpret_cast<const int*>(d + L.o_en);
    A.K.v = reinterpret_cast<double*>(d + L.o_v);
    A.K.W = reinterpret_cast<double*>(d + L.o_W);
    A.K.chi2 = reinterpret_cast<double*>(d + L.o_chi2);
    A.K.D = reinterpret_cast<double*>(d + L.o_D);
    A.K.L = reinterpret_cast<double*>(d + L.o_L);
    A.K.U = reinterpret_cast<double*>(d + L.o_U);
    A.K.R = reinterpret_cast<double*>(d + L.o_R);
    A.K.R0 = reinterpret_cast<double*>(d + L.o_R0);
    A.K.x = reinterpret_cast<double*>(d + L.o_x);
    A.problem = reinterpret_cast<const msorb_inertial_problem*>(d + L.o_prob);
    A.result = reinterpret_cast<msorb_inertial_result*>(d + L.o_res);
    hipStream_t s = scr.s;
    float ms = 0;
    hipError_t e = msorb::small_copy(d, h, L.in_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && elapsed_ms) e = hipEventRecord(scr.ev[0], s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(inertial_opt_kernel, dim3(1), dim3(kThreads), 0, s, A);
        e = hipGetLastError();
    }
    if (e == hipSuccess && elapsed_ms) e = hipEventRecord(scr.ev[1], s);
    if (e == hipSuccess) e = msorb::small_copy(h + L.o_res, d + L.o_res, L.out_end - L.o_res, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess && elapsed_ms) e = hipEventElapsedTime(&ms, scr.ev[0], scr.ev[1]);
    if (e != hipSuccess) {
        set_last_error(std::string("inertial_optimization: ") + hipGetErrorString(e));
        scr.release();
        return MSORB_E_HIP;
    }
    std::memcpy(r, h + L.o_res, sizeof(*r));
    if (nk) std::memcpy(v_out, h + L.o_v, nk * 24);
    if (ne && edge_chi2) std::memcpy(edge_chi2, h + L.o_chi2, ne * 8);
    if (elapsed_ms) *elapsed_ms = ms;
    return MSORB_OK;
}
