// Optimizer::LocalBundleAdjustment (src/Optimizer.cc:1040-1407) and Optimizer::BundleAdjustment (:60-364, reached through
// GlobalBundleAdjustemnt, :51-58) for pinhole KeyFrames without a second camera: g2o's Levenberg-Marquardt over KeyFrame poses and
// map points with the points eliminated by the Schur complement (core/block_solver.hpp:354-486), in double.  Both entries run ONE
// engine, ba_engine below; what the reference does differently in the two is the Entry struct.  DESIGN.md sections 10 and 16 have
// the whole story.
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
//               reduced system adds W_a D^-1 W_b^T over the pair's list and one per KeyFrame adds W D^-1 bl; the dense
//               6 Kf x 6 Kf system is factored (L D L^T, no pivoting, no square root) and substituted, by ONE workgroup
//               (ba_solve_kernel) under msorb_local_ba and by the blocked kernels of ldlt_blocked.h under msorb_bundle_adjustment:
//               the same bits either way, see Entry::one_workgroup_solve; one thread per vertex applies the update to a second
//               copy of the state (push / pop is which copy is current) and returns its share of computeScale; the errors at the
//               trial state; a one-workgroup reduction of the cost and the scale.
//
// The square of the reduced system is zeroed before every trial's Schur launch: the Schur kernel writes the listed block pairs only
// and the factorisation, which is in place, fills the rest in.  A rejected trial therefore rebuilds S from Hpp and the lists.
//
// No floating-point atomics: every sum walks an index list of local_ba_plan.h in a fixed order, two runs return the same bits.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/msorb.h"
#include "ba_kernels_device.h"
#include "hip_host.h"
#include "ldlt_blocked.h"
#include "local_ba_plan.h"

using msorb::set_last_error;
using msorb::ThreadScratch;
using namespace msorb::ba;
namespace ldlt = msorb::ldlt;

namespace {

// Free KeyFrames.  Local: the reduced system is at most 768 x 768, four columns of which are ba_solve_kernel's LDS; the host
// template hands a larger window back to the reference path.  Global: S is 6144^2 doubles = 302 MB.
constexpr int kLocalCapacity = 128, kGlobalCapacity = 1024;
constexpr int kMaxN = 6 * kLocalCapacity;
constexpr int kSolveThreads = 1024;

// What the reference does differently in LocalBundleAdjustment and in BundleAdjustment.
struct Entry {
    const char* name;          // "local_ba" / "bundle_adjustment": error strings
    int capacity;
    float d_mono;              // thHuber2D: (float)sqrt(5.991) at :1190, (float)sqrt(5.99) at :128
    int robust;                // local: always (:1186-1191); global: bRobust (:174, :206)
    int iterations;
    bool one_workgroup_solve;  // ba_solve_kernel instead of ldlt::launch.  Both return the same bits (tests/test_ldlt_gpu.py, and the
                               // 128-KeyFrame scene of tests/test_bundle_adjustment_gpu.py through both entries); the blocked solve is
                               // 1.2 / 2.0 / 5.1 times faster for the whole call at 20 / 40 / 80 free KeyFrames but its four
                               // launches cost a call of 2 free KeyFrames 0.05 ms (0.96 against 0.91 ms), so local keeps the one
                               // launch until small systems take fewer
    bool local;                // *r zeroed first; the early returns of :1098-1102 and :1323-1325; the classification of :1331-1373;
                               // every point is a vertex (global: a point without an edge is none, :261-263)
    uint8_t* edge_outlier;     // local's output, [E]
    uint8_t* point_included;   // global's output, [P]
};

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

// :1331-1373: computeError at the final estimate, float fChi2 > 5.991 / 7.815 (double literals) or !isDepthPositive()
__global__ __launch_bounds__(kEdgeThreads) void ba_classify_kernel(const BaDev A, int s) {
    const int e = blockIdx.x * kEdgeThreads + threadIdx.x;
    if (e >= A.E) return;
    int k, p;
    const EdgeGeom g = edge_geom(A, s, e, k, p);
    const double c = (double)(float)g.chi2;
    A.outlier[e] = (c > (g.stereo ? 7.815 : 5.991) || !(g.z > 0.0)) ? 1 : 0;
}

int stage_ms(float ms[4]) {
    if (!ms) return MSORB_E_ARG;
    for (int i = 0; i < kStages; i++) ms[i] = g_stages.ms[i];
    return stages_on() ? MSORB_OK : MSORB_E_ARG;
}

int ba_engine(const Entry& f, int device, int n_kf, const msorb_ba_keyframe* kfs, int n_points, const float* pos_w, int n_edges,
              const int* edge_kf, const int* edge_point, const float* xy, const float* u_right, const float* inv_sigma2,
              const volatile int* stop_flag, float* kf_qt_out, double* kf_qt_d, float* pos_out, double* pos_d, msorb_ba_result* r,
              float* elapsed_ms) {
    if (elapsed_ms) *elapsed_ms = 0;
    if (!r || n_kf < 0 || n_points < 0 || n_edges < 0 || f.iterations < 0) return MSORB_E_ARG;
    if ((n_kf > 0 && (!kfs || !kf_qt_out)) || (n_points > 0 && (!pos_w || !pos_out || (!f.local && !f.point_included))) ||
        (n_edges > 0 && (!edge_kf || !edge_point || !xy || !u_right || !inv_sigma2 || (f.local && !f.edge_outlier))))
        return MSORB_E_ARG;
    if (f.local) std::memset(r, 0, sizeof *r);   // (global leaves every output untouched until the capacity checks have passed)
    const int K = n_kf, P = n_points, E = n_edges;
    const std::string name = std::string(f.name) + ": ";
    static thread_local std::vector<int> fixed;
    static thread_local msorb::LocalBaPlan plan;
    fixed.resize((size_t)K);
    for (int k = 0; k < K; k++) fixed[k] = kfs[k].fixed != 0;
    switch (msorb::build_local_ba_plan(K, fixed.data(), P, E, edge_kf, edge_point, plan)) {
        case msorb::kPlanIndexOutOfRange: set_last_error(name + "an edge names a KeyFrame or a point out of range"); return MSORB_E_ARG;
        case msorb::kPlanNotPointMajor: set_last_error(name + "the edges are not point-major"); return MSORB_E_ARG;
        default: break;
    }
    const int Kf = plan.Kf, n = 6 * Kf;
    if (Kf > f.capacity) {
        set_last_error(name + "more free KeyFrames than msorb_" + f.name + "_capacity()");
        return MSORB_E_CAPACITY;
    }
    if (f.local && (Kf == K || (stop_flag && *stop_flag))) {   // :1098-1102, :1323-1325: nothing touched, the outputs are the inputs
        r->status = Kf == K ? 1 : 2;
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
        if (E) std::memset(f.edge_outlier, 0, (size_t)E);
        return MSORB_OK;
    }
    if (int rc = msorb::require_device(device)) return rc;

    // ---- the device block: [uploaded | state and workspaces | results]
    const int n_pairs = (int)plan.pair_i.size(), n_blocks = (E + kEdgeThreads - 1) / kEdgeThreads;
    const size_t n_entries = plan.pair_a.size(), n_out = f.local ? (size_t)E : 0;
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
    const size_t o_ws = c.take(f.one_workgroup_solve ? 0 : ldlt::workspace_doubles(n) * 8);
    const size_t o_pc = c.take((size_t)n_blocks * 8), o_pv = c.take(((size_t)Kf + P) * 8);
    const size_t o_res = c.take(sizeof(BaRes)), o_out = c.take(n_out);
    const size_t dev_bytes = c.at;
    // pinned: the upload, then [res | pose | points | outlier] for the read-backs
    Carve hc;
    hc.at = in_bytes;
    const size_t h_res = hc.take(sizeof(BaRes)), h_pose = hc.take((size_t)K * 56), h_pt = hc.take((size_t)P * 24), h_out = hc.take(n_out);
    static thread_local ThreadScratch scr(true, 2);
    if (dev_bytes > scr.d.n) {   // the block has to grow (by 1.5x): a reduced system that does not fit is a matter of capacity
        if (hipSetDevice(device) != hipSuccess) return MSORB_E_HIP;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && dev_bytes + dev_bytes / 2 + 16 > free_b + (scr.device == device ? scr.d.n : 0)) {
            set_last_error(name + "the device has no room for the reduced system");
            return MSORB_E_CAPACITY;
        }
    }
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
    {   // :1134, :1150 / :138, :202: the float pose widened, SE3Quat's constructor normalises (se3quat.h:62-64); the point widened
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
    A.outlier = f.local ? d + o_out : nullptr;
    A.d_mono = f.d_mono;
    A.d_stereo = (float)std::sqrt(7.815);
    A.robust = f.robust;
    ldlt::Work W{};
    W.n = n; W.S = A.S; W.b = A.bs; W.x = A.x;
    ldlt::carve_workspace(W, dp(o_ws));
    W.ok = &A.res->solver_ok;

    hipError_t err = hipSuccess;
    auto fail = [&](const char* what) {
        set_last_error(name + what + ": " + hipGetErrorString(err));
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
    std::memset(r, 0, sizeof *r);   // (global's first write of it)
    auto stopped = [&] { return stop_flag && *stop_flag; };   // SparseOptimizer::terminate
    bool ok = E > 0;   // without an edge there is nothing to optimise: zero iterations, the estimates as they came
    for (int it = 0; it < f.iterations && !stopped() && ok; it++) {   // sparse_optimizer.cpp:376
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
            if (f.one_workgroup_solve) BA_LAUNCH(ba_solve_kernel, n ? 1 : 0, kSolveThreads, A);
            else BA_TRY(ldlt::launch(W, s));
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
    if (f.local) BA_LAUNCH(ba_classify_kernel, n_blocks, kEdgeThreads, A, cur);
    if (elapsed_ms) BA_TRY(hipEventRecord(scr.ev[1], s));
    BA_TRY(hipMemcpyAsync(h + h_pose, d + (cur ? o_pose1 : o_pose0), (size_t)K * 56, hipMemcpyDeviceToHost, s));
    if (P) BA_TRY(hipMemcpyAsync(h + h_pt, d + (cur ? o_pt1 : o_pt0), (size_t)P * 24, hipMemcpyDeviceToHost, s));
    if (n_out) BA_TRY(hipMemcpyAsync(h + h_out, d + o_out, n_out, hipMemcpyDeviceToHost, s));
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
            kf_qt_out[7 * (size_t)k + a] = fx ? in : (float)hp[7 * (size_t)k + a];   // :1393 / :284-288
            if (kf_qt_d) kf_qt_d[7 * (size_t)k + a] = fx ? (double)in : hp[7 * (size_t)k + a];
        }
    const double* hx = reinterpret_cast<const double*>(h + h_pt);
    for (int p = 0; p < P; p++) {
        const bool in = f.local || plan.point_begin[p + 1] > plan.point_begin[p];   // :261-263: without an edge it is no vertex
        if (!f.local) f.point_included[p] = in ? 1 : 0;
        for (int a = 0; a < 3; a++) {
            const size_t i = 3 * (size_t)p + a;
            pos_out[i] = in ? (float)hx[i] : pos_w[i];   // :1402 / :356-362
            if (pos_d) pos_d[i] = in ? hx[i] : (double)pos_w[i];
        }
    }
    int n_outliers = 0;
    for (size_t e = 0; e < n_out; e++) { f.edge_outlier[e] = h[h_out + e]; n_outliers += f.edge_outlier[e] != 0; }
    r->status = 0;
    r->iterations = iterations;
    r->trials = trials;
    r->rejected_trials = rejected;
    r->n_outliers = n_outliers;
    r->lambda_final = lambda;
    return MSORB_OK;
}

}  // namespace

extern "C" int msorb_local_ba_capacity(void) { return kLocalCapacity; }
extern "C" int msorb_bundle_adjustment_capacity(void) { return kGlobalCapacity; }
extern "C" int msorb_local_ba_stage_ms(float ms[4]) { return stage_ms(ms); }
extern "C" int msorb_bundle_adjustment_stage_ms(float ms[4]) { return stage_ms(ms); }

extern "C" int msorb_local_ba(int device, int n_kf, const msorb_ba_keyframe* kfs, int n_points, const float* pos_w, int n_edges,
                              const int* edge_kf, const int* edge_point, const float* xy, const float* u_right, const float* inv_sigma2,
                              int max_iterations, const volatile int* stop_flag, float* kf_qt_out, double* kf_qt_d, float* pos_out,
                              double* pos_d, uint8_t* edge_outlier, msorb_ba_result* r, float* elapsed_ms) {
    const Entry f{"local_ba", kLocalCapacity, (float)std::sqrt(5.991), 1, max_iterations, true, true, edge_outlier, nullptr};
    return ba_engine(f, device, n_kf, kfs, n_points, pos_w, n_edges, edge_kf, edge_point, xy, u_right, inv_sigma2, stop_flag, kf_qt_out,
                     kf_qt_d, pos_out, pos_d, r, elapsed_ms);
}

extern "C" int msorb_bundle_adjustment(int device, int n_kf, const msorb_ba_keyframe* kfs, int n_points, const float* pos_w,
                                       int n_edges, const int* edge_kf, const int* edge_point, const float* xy, const float* u_right,
                                       const float* inv_sigma2, int n_iterations, int robust, const volatile int* stop_flag,
                                       float* kf_qt_out, double* kf_qt_d, float* pos_out, double* pos_d, uint8_t* point_included,
                                       msorb_ba_result* r, float* elapsed_ms) {
    const Entry f{"bundle_adjustment", kGlobalCapacity, (float)std::sqrt(5.99), robust != 0, n_iterations, false, false, nullptr, point_included};
    return ba_engine(f, device, n_kf, kfs, n_points, pos_w, n_edges, edge_kf, edge_point, xy, u_right, inv_sigma2, stop_flag, kf_qt_out,
                     kf_qt_d, pos_out, pos_d, r, elapsed_ms);
}
