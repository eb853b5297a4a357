// Optimizer::BundleAdjustment (src/Optimizer.cc:60-364, reached through GlobalBundleAdjustemnt, :51-58) for pinhole KeyFrames
// without a second camera: the kernels of ba_kernels_device.h under g2o's Levenberg loop, as local_ba.hip drives them, with the
// reduced system solved by the blocked, multi-workgroup L D L^T of ldlt_blocked.h.  DESIGN.md section 16 has the whole story.
//
// What differs from msorb_local_ba restates the reference: bRobust is a switch (:174, :206), the iteration count is the caller's
// (:269), there is no early return without a fixed KeyFrame and none for a stop flag that is already set (optimize() then makes zero
// iterations), no classification follows, and a point without an edge is no vertex (:261-263).
//
// The square of the reduced system is zeroed before every trial's Schur launch: the Schur kernel writes the listed block pairs only
// and the factorisation, which is in place, fills the rest in.  A rejected trial therefore rebuilds S from Hpp and the lists.
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
constexpr int kCapacity = 1024;   // free KeyFrames: S is 6144^2 doubles = 302 MB
}

extern "C" int msorb_bundle_adjustment_capacity(void) { return kCapacity; }

extern "C" int msorb_bundle_adjustment_stage_ms(float ms[4]) {
    if (!ms) return MSORB_E_ARG;
    for (int i = 0; i < kStages; i++) ms[i] = g_stages.ms[i];
    return stages_on() ? MSORB_OK : MSORB_E_ARG;
}

extern "C" int msorb_bundle_adjustment(int device, int n_kf, const msorb_ba_keyframe* kfs, int n_points, const float* pos_w,
                                       int n_edges, const int* edge_kf, const int* edge_point, const float* xy, const float* u_right,
                                       const float* inv_sigma2, int n_iterations, int robust, const volatile int* stop_flag,
                                       float* kf_qt_out, double* kf_qt_d, float* pos_out, double* pos_d, uint8_t* point_included,
                                       msorb_ba_result* r, float* elapsed_ms) {
    if (elapsed_ms) *elapsed_ms = 0;
    if (!r || n_kf < 0 || n_points < 0 || n_edges < 0 || n_iterations < 0) return MSORB_E_ARG;
    if ((n_kf > 0 && (!kfs || !kf_qt_out)) || (n_points > 0 && (!pos_w || !pos_out || !point_included)) ||
        (n_edges > 0 && (!edge_kf || !edge_point || !xy || !u_right || !inv_sigma2)))
        return MSORB_E_ARG;
    const int K = n_kf, P = n_points, E = n_edges;
    static thread_local std::vector<int> fixed;
    static thread_local msorb::LocalBaPlan plan;
    fixed.resize((size_t)K);
    for (int k = 0; k < K; k++) fixed[k] = kfs[k].fixed != 0;
    switch (msorb::build_local_ba_plan(K, fixed.data(), P, E, edge_kf, edge_point, plan)) {
        case msorb::kPlanIndexOutOfRange: set_last_error("bundle_adjustment: an edge names a KeyFrame or a point out of range"); return MSORB_E_ARG;
        case msorb::kPlanNotPointMajor: set_last_error("bundle_adjustment: the edges are not point-major"); return MSORB_E_ARG;
        default: break;
    }
    const int Kf = plan.Kf, n = 6 * Kf;
    if (Kf > kCapacity) {
        set_last_error("bundle_adjustment: more free KeyFrames than msorb_bundle_adjustment_capacity()");
        return MSORB_E_CAPACITY;
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
    const size_t o_ws = c.take(ldlt::workspace_doubles(n) * 8);
    const size_t o_pc = c.take((size_t)n_blocks * 8), o_pv = c.take(((size_t)Kf + P) * 8);
    const size_t o_res = c.take(sizeof(BaRes));
    const size_t dev_bytes = c.at;
    // pinned: the upload, then [res | pose | points] for the read-backs
    Carve hc;
    hc.at = in_bytes;
    const size_t h_res = hc.take(sizeof(BaRes)), h_pose = hc.take((size_t)K * 56), h_pt = hc.take((size_t)P * 24);
    static thread_local ThreadScratch scr(true, 2);
    if (dev_bytes > scr.d.n) {   // the block has to grow (by 1.5x): a reduced system that does not fit is a matter of capacity
        if (hipSetDevice(device) != hipSuccess) return MSORB_E_HIP;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && dev_bytes + dev_bytes / 2 + 16 > free_b + (scr.device == device ? scr.d.n : 0)) {
            set_last_error("bundle_adjustment: the device has no room for the reduced system");
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
    {   // :138, :202: the float pose widened, SE3Quat's constructor normalises (se3quat.h:62-64); the point widened
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
    A.outlier = nullptr;   // no classification here
    A.d_mono = (float)std::sqrt(5.99);      // :128-129: thHuber2D is sqrt(5.99) HERE (5.991 in LocalBundleAdjustment), thHuber3D sqrt(7.815)
    A.d_stereo = (float)std::sqrt(7.815);
    A.robust = robust != 0;
    ldlt::Work W{};
    W.n = n; W.S = A.S; W.b = A.bs; W.x = A.x;
    ldlt::carve_workspace(W, dp(o_ws));
    W.ok = &A.res->solver_ok;

    hipError_t err = hipSuccess;
    auto fail = [&](const char* what) {
        set_last_error(std::string("bundle_adjustment: ") + what + ": " + hipGetErrorString(err));
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
    std::memset(r, 0, sizeof *r);
    auto stopped = [&] { return stop_flag && *stop_flag; };   // SparseOptimizer::terminate
    bool ok = E > 0;   // without an edge there is nothing to optimise: zero iterations, the estimates as they came
    for (int it = 0; it < n_iterations && !stopped() && ok; it++) {   // sparse_optimizer.cpp:376
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
            BA_TRY(ldlt::launch(W, s));
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
    if (elapsed_ms) BA_TRY(hipEventRecord(scr.ev[1], s));
    BA_TRY(hipMemcpyAsync(h + h_pose, d + (cur ? o_pose1 : o_pose0), (size_t)K * 56, hipMemcpyDeviceToHost, s));
    if (P) BA_TRY(hipMemcpyAsync(h + h_pt, d + (cur ? o_pt1 : o_pt0), (size_t)P * 24, hipMemcpyDeviceToHost, s));
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
            kf_qt_out[7 * (size_t)k + a] = fx ? in : (float)hp[7 * (size_t)k + a];   // :284-288
            if (kf_qt_d) kf_qt_d[7 * (size_t)k + a] = fx ? (double)in : hp[7 * (size_t)k + a];
        }
    const double* hx = reinterpret_cast<const double*>(h + h_pt);
    for (int p = 0; p < P; p++) {
        const bool in = plan.point_begin[p + 1] > plan.point_begin[p];   // :261-263: without an edge it is no vertex
        point_included[p] = in ? 1 : 0;
        for (int a = 0; a < 3; a++) {
            const size_t i = 3 * (size_t)p + a;
            pos_out[i] = in ? (float)hx[i] : pos_w[i];   // :356-362
            if (pos_d) pos_d[i] = in ? hx[i] : (double)pos_w[i];
        }
    }
    r->status = 0;
    r->iterations = iterations;
    r->trials = trials;
    r->rejected_trials = rejected;
    r->n_outliers = 0;
    r->lambda_final = lambda;
    return MSORB_OK;
}
