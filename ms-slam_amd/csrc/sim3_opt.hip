// Optimizer::OptimizeSim3 (src/Optimizer.cc:1986-2242, :2244-2429) after its gathering loops, for two pinhole cameras: one 7-DoF
// Sim3 vertex over 2N binary edges whose points are fixed, the whole routine in ONE launch, in double like g2o.  The arithmetic
// is sim3_opt_device.h, the same text a host compiler reads; this file is the executor that spreads it over a workgroup.
//
// One workgroup of 256 threads owns a problem (blockIdx.x = problem), as in pose_opt.hip.  Thread t owns the pairs t, t + 256, ...:
// up to kPerThread = 2 of them live in registers as the reference's floats (N <= kResident = 512) with their two chi2 and their
// flag; a longer problem walks the same indices in global memory, its per-pair state in the output arrays.  Both forms add in
// the same order.
//
// A linearisation needs the estimate perturbed by +-1e-9 along each of the 7 directions through oplus, and the inverse of each
// for the e21 edges: 28 transforms that are the same for every edge.  Threads 0..13 compute one perturbed estimate and its
// inverse each and put them in LDS (1792 bytes); after one barrier every thread reads them from there (all lanes read one address:
// a broadcast).  The table is written again only after the reductions of the step, whose barriers every reader has passed.
// The map over the pairs then adds, pair by pair, e12's and e21's 36 terms (28 of H's upper triangle, 7 of b, the cost), and
// ONE reduction follows: block_sum of pose_opt.hip with 36 sums (per thread ascending, xor butterfly 32..1 in a wavefront, the
// four wavefronts in ascending order through a double-buffered LDS block).  Every thread then solves the 7x7 system and updates
// the estimate redundantly.  A trial is a second map (errors only) and a one-value reduction.  No atomics: two runs give the
// same bits.  Every trip count comes from reduced values that all threads hold with equal bits, so every thread reaches every
// barrier.  The 7x7 solve and Sim3(update) stay out of line on the device (sim3_opt_device.h): inlined next to the 36 sums they
// overflow the register file.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/msorb.h"
#include "hip_host.h"
#include "matcher_host.h"
#include "sim3_opt_device.h"

namespace msorb {
hipError_t small_copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s);   // orb_kernels.hip
}
using msorb::set_last_error;
using msorb::ThreadScratch;
using msorb::up16;
using namespace msorb::sim3opt;

namespace {

constexpr int kThreads = 256, kPerThread = 2, kResident = kThreads * kPerThread, kWaves = kThreads / 64;

struct Sim3ProblemDev {
    msorb_sim3_opt_problem p;
    int pair0;   // first pair of the problem in the flat arrays
    int pad;
};
static_assert(sizeof(msorb_sim3_opt_problem) == 128 && sizeof(msorb_sim3_opt_result) == 96, "the records of include/msorb.h as the Python mirror lays them out");
static_assert(sizeof(Sim3) == 64, "the LDS table");

struct Sim3Args {
    const Sim3ProblemDev* prob;
    const float *P1, *P2, *o1, *o2, *w1, *w2;   // per pair
    double* chi2;     // 2 per pair: out, and the state of the problems with n > kResident
    uint8_t* bad;     // per pair: out, and the state of the problems with n > kResident
    msorb_sim3_opt_result* result;
};

__device__ inline Pair load_pair(const Sim3Args& A, size_t i) {
    Pair p;
    for (int k = 0; k < 3; k++) { p.P1[k] = A.P1[3 * i + k]; p.P2[k] = A.P2[3 * i + k]; }
    for (int k = 0; k < 2; k++) { p.o1[k] = A.o1[2 * i + k]; p.o2[k] = A.o2[2 * i + k]; }
    p.w1 = A.w1[i]; p.w2 = A.w2[i];
    return p;
}

template <bool RES>
struct BlockExec {
    const Sim3Args& A;
    const int pair0, n;
    double* const lds_sum;   // 2 blocks of kWaves * kSums
    Sim3* const lds_tab;     // 2 * kPerturbed
    int buf = 0;
    Pair pr[RES ? kPerThread : 1];
    double chi2[RES ? kPerThread : 1][2];
    uint8_t flag[RES ? kPerThread : 1];

    __device__ BlockExec(const Sim3Args& a, int p0, int n_, double* ls, Sim3* lt) : A(a), pair0(p0), n(n_), lds_sum(ls), lds_tab(lt) {
        if constexpr (RES) {
#pragma unroll
            for (int k = 0; k < kPerThread; k++) {
                const int i = threadIdx.x + k * kThreads;
                pr[k] = i < n ? load_pair(A, (size_t)pair0 + i) : Pair{};
                chi2[k][0] = chi2[k][1] = 0;
                flag[k] = 0;
            }
        } else {
            for (int i = threadIdx.x; i < n; i += kThreads) {
                A.chi2[2 * ((size_t)pair0 + i)] = 0; A.chi2[2 * ((size_t)pair0 + i) + 1] = 0;
                A.bad[(size_t)pair0 + i] = 0;
            }
        }
    }

    // f over the thread's pairs in ascending index
    template <typename F>
    __device__ inline void for_each_pair(F f) {
        if constexpr (RES) {
#pragma unroll
            for (int k = 0; k < kPerThread; k++)
                if ((int)threadIdx.x + k * kThreads < n) f(pr[k], chi2[k], flag[k]);
        } else {
            for (int i = threadIdx.x; i < n; i += kThreads) {
                const size_t g = (size_t)pair0 + i;
                const Pair p = load_pair(A, g);
                double c[2] = {A.chi2[2 * g], A.chi2[2 * g + 1]};
                uint8_t fl = A.bad[g];
                f(p, c, fl);
                A.chi2[2 * g] = c[0]; A.chi2[2 * g + 1] = c[1];
                A.bad[g] = fl;
            }
        }
    }

    // block_sum of pose_opt.hip: every thread returns with the same bits; the two LDS blocks alternate, so the one barrier also
    // protects the block of the reduction before the last
    template <int N>
    __device__ inline void sum(double* v) {
        double* lds = lds_sum + (buf ^= 1) * kWaves * kSums;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
            for (int i = 0; i < N; i++) v[i] += msorb::se3::shfl_xor_f64(v[i], off);
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

    __device__ inline const Sim3* perturbed(const Sim3& S, bool fix_scale) {
        if (threadIdx.x < kPerturbed) sim3_perturbed(S, fix_scale, threadIdx.x, lds_tab[threadIdx.x], lds_tab[kPerturbed + threadIdx.x]);
        __syncthreads();
        return lds_tab;
    }

    __device__ inline bool leader() const { return threadIdx.x == 0; }

    __device__ inline void store() {
        if constexpr (RES) {
#pragma unroll
            for (int k = 0; k < kPerThread; k++) {
                const int i = threadIdx.x + k * kThreads;
                if (i < n) {
                    const size_t g = (size_t)pair0 + i;
                    A.bad[g] = flag[k];
                    A.chi2[2 * g] = chi2[k][0]; A.chi2[2 * g + 1] = chi2[k][1];
                }
            }
        }
    }
};

template <bool RES>
__device__ void sim3_opt_problem(const Sim3Args& A, double* lds_sum, Sim3* lds_tab) {
    const Sim3ProblemDev P = A.prob[blockIdx.x];
    BlockExec<RES> ex(A, P.pair0, P.p.n, lds_sum, lds_tab);
    optimize_sim3(ex, P.p, A.result[blockIdx.x]);
    ex.store();
}

__global__ __launch_bounds__(kThreads) void sim3_opt_kernel(const Sim3Args A) {
    __shared__ double lds_sum[2 * kWaves * kSums];
    __shared__ Sim3 lds_tab[2 * kPerturbed];
    if (A.prob[blockIdx.x].p.n <= kResident) sim3_opt_problem<true>(A, lds_sum, lds_tab);
    else sim3_opt_problem<false>(A, lds_sum, lds_tab);
}

// Staging: [problems | P1 | P2 | o1 | o2 | w1 | w2] up, [results | bad | chi2] down.
struct Staged {
    size_t o_prob, o_P1, o_P2, o_o1, o_o2, o_w1, o_w2, in_bytes, o_res, o_bad, o_chi2, bytes;
    Staged(int np, size_t tot) {
        o_prob = 0;
        o_P1 = up16((size_t)np * sizeof(Sim3ProblemDev));
        o_P2 = o_P1 + up16(tot * 12);
        o_o1 = o_P2 + up16(tot * 12);
        o_o2 = o_o1 + up16(tot * 8);
        o_w1 = o_o2 + up16(tot * 8);
        o_w2 = o_w1 + up16(tot * 4);
        in_bytes = o_w2 + up16(tot * 4);
        o_res = in_bytes;
        o_bad = o_res + up16((size_t)np * sizeof(msorb_sim3_opt_result));
        o_chi2 = o_bad + up16(tot);
        bytes = o_chi2 + up16(tot * 16);
    }
};

}  // namespace

extern "C" int msorb_sim3_optimization_capacity(void) { return kResident; }

extern "C" int msorb_sim3_optimization_batch(int device, int n_problems, const msorb_sim3_opt_problem* problems, const int* pair_offset,
                                             const float* P1c, const float* P2c, const float* obs1, const float* obs2,
                                             const float* inv_sigma2_1, const float* inv_sigma2_2, uint8_t* bad_out, double* chi2_out,
                                             msorb_sim3_opt_result* results, float* elapsed_ms) {
    if (n_problems < 0 || (n_problems > 0 && (!problems || !pair_offset || !results))) return MSORB_E_INVALID;
    if (n_problems == 0) { if (elapsed_ms) *elapsed_ms = 0; return MSORB_OK; }
    if (pair_offset[0] != 0) { set_last_error("sim3_optimization_batch: pair_offset[0] must be 0"); return MSORB_E_INVALID; }
    for (int i = 0; i < n_problems; i++) {
        const msorb_sim3_opt_problem& p = problems[i];
        if (p.n < 0 || pair_offset[i + 1] - pair_offset[i] != p.n) {
            set_last_error("sim3_optimization_batch: pair_offset does not match the problems' n");
            return MSORB_E_INVALID;
        }
        if (p.its[0] < 1 || p.its[1] < 1 || p.its[2] < 1) {
            set_last_error("sim3_optimization_batch: an entry of its is below 1");
            return MSORB_E_INVALID;
        }
    }
    const size_t total = (size_t)pair_offset[n_problems];
    if (total > 0 && (!P1c || !P2c || !obs1 || !obs2 || !inv_sigma2_1 || !inv_sigma2_2 || !bad_out)) return MSORB_E_INVALID;
    if (int rc = msorb::require_device(device)) return rc;
    const Staged L(n_problems, total);
    static thread_local ThreadScratch scr(true, 3);
    if (int rc = scr.acquire(device, L.bytes, L.bytes)) return rc;
    uint8_t *const h = scr.h.p, *const d = scr.d.p;
    Sim3ProblemDev* hp = reinterpret_cast<Sim3ProblemDev*>(h + L.o_prob);
    for (int i = 0; i < n_problems; i++) { hp[i].p = problems[i]; hp[i].pair0 = pair_offset[i]; hp[i].pad = 0; }
    if (total) {
        std::memcpy(h + L.o_P1, P1c, total * 12);
        std::memcpy(h + L.o_P2, P2c, total * 12);
        std::memcpy(h + L.o_o1, obs1, total * 8);
        std::memcpy(h + L.o_o2, obs2, total * 8);
        std::memcpy(h + L.o_w1, inv_sigma2_1, total * 4);
        std::memcpy(h + L.o_w2, inv_sigma2_2, total * 4);
    }
    Sim3Args A{};
    A.prob = reinterpret_cast<const Sim3ProblemDev*>(d + L.o_prob);
    A.P1 = reinterpret_cast<const float*>(d + L.o_P1);
    A.P2 = reinterpret_cast<const float*>(d + L.o_P2);
    A.o1 = reinterpret_cast<const float*>(d + L.o_o1);
    A.o2 = reinterpret_cast<const float*>(d + L.o_o2);
    A.w1 = reinterpret_cast<const float*>(d + L.o_w1);
    A.w2 = reinterpret_cast<const float*>(d + L.o_w2);
    A.result = reinterpret_cast<msorb_sim3_opt_result*>(d + L.o_res);
    A.bad = d + L.o_bad;
    A.chi2 = reinterpret_cast<double*>(d + L.o_chi2);
    hipStream_t s = scr.s;
    float ms = 0;
    hipError_t e = msorb::small_copy(d, h, L.in_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && elapsed_ms) e = hipEventRecord(scr.ev[0], s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(sim3_opt_kernel, dim3(n_problems), dim3(kThreads), 0, s, A);
        e = hipGetLastError();
    }
    if (e == hipSuccess && elapsed_ms) e = hipEventRecord(scr.ev[1], s);
    if (e == hipSuccess) e = msorb::small_copy(h + L.o_res, d + L.o_res, L.bytes - L.o_res, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess && elapsed_ms) e = hipEventElapsedTime(&ms, scr.ev[0], scr.ev[1]);
    if (e != hipSuccess) {
        set_last_error(std::string("sim3_optimization: ") + hipGetErrorString(e));
        scr.release();
        return MSORB_E_HIP;
    }
    std::memcpy(results, h + L.o_res, (size_t)n_problems * sizeof(msorb_sim3_opt_result));
    if (total) {
        std::memcpy(bad_out, h + L.o_bad, total);
        if (chi2_out) std::memcpy(chi2_out, h + L.o_chi2, total * 16);
    }
    if (elapsed_ms) *elapsed_ms = ms;
    return MSORB_OK;
}
