// Optimizer::LocalBundleAdjustment (src/Optimizer.cc:1040-1407), Optimizer::BundleAdjustment (:60-364, reached through
// GlobalBundleAdjustemnt, :51-58) and the welding LocalBundleAdjustment of a map merge (:3494-3915) for pinhole KeyFrames without a
// second camera: g2o's Levenberg-Marquardt over KeyFrame poses and map points with the points eliminated by the Schur complement
// (core/block_solver.hpp:354-486), in double.  All entries run ONE engine, ba_engine below; what the reference does differently in
// them is the Entry struct.  DESIGN.md sections 10, 16 and 27 have the whole story.
//
// One optimize() of g2o is `run` inside the engine: it starts from the state the previous run left, with lambda, ni and the count
// of bad iterations initialised anew at its iteration 0.  The welding entry runs it twice: optimize(5) with Huber kernels on every
// edge, a classification that puts edges on level 1, and optimize(10) without kernels over the level-0 edges alone.  The second
// graph is made on the host (one read-back of E bytes): the level-0 edges compacted, a free KeyFrame that no level-0 edge reaches
// marked fixed, a new plan.  So a vertex that is not in the second problem is not written by it, and the kernels do not know of levels.
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

// What the reference does differently in LocalBundleAdjustment, in BundleAdjustment and in the welding LocalBundleAdjustment.
struct Entry {
    const char* name;          // "local_ba" / "bundle_adjustment" / "welding_ba": error strings
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
    // the welding bundle adjustment (:3494-3915): no "no fixed KeyFrame" return; optimize(5) robust, classification into levels
    // (:3726-3753), optimize(10) over level 0 without kernels, classification (:3769-3803).  `robust` is round 1's; `iterations` is not read.
    bool welding = false;
    uint8_t* edge_level1 = nullptr;            // [E]
    msorb_welding_ba_result* wr = nullptr;
};

// Where one graph's index lists and edge arrays lie inside an upload, relative to its start.  The welding entry has two graphs:
// one function lays both out, one fills in a plan's lists, one points a BaDev at them.
struct GraphLayout {
    size_t free_of_kf, kf_of_free, edge_kf, edge_pt, point_begin, kf_begin, kf_edge, pair_begin, pair_i, pair_j, pair_a, pair_b, xy, ur, w;
};
// room for a graph of K KeyFrames, P points and E edges with the lists of `plan`, or of any plan over a subset of its edges
GraphLayout carve_graph(Carve& c, int K, int P, int E, const msorb::LocalBaPlan& plan) {
    const size_t Kf = (size_t)plan.Kf, n_pairs = plan.pair_i.size(), n_entries = plan.pair_a.size();
    GraphLayout g;
    g.free_of_kf = c.take((size_t)K * 4); g.kf_of_free = c.take(Kf * 4);
    g.edge_kf = c.take((size_t)E * 4); g.edge_pt = c.take((size_t)E * 4); g.point_begin = c.take(((size_t)P + 1) * 4);
    g.kf_begin = c.take((Kf + 1) * 4); g.kf_edge = c.take(plan.kf_edge.size() * 4);
    g.pair_begin = c.take((n_pairs + 1) * 4); g.pair_i = c.take(n_pairs * 4); g.pair_j = c.take(n_pairs * 4);
    g.pair_a = c.take(n_entries * 4); g.pair_b = c.take(n_entries * 4);
    g.xy = c.take((size_t)E * 8); g.ur = c.take((size_t)E * 4); g.w = c.take((size_t)E * 4);
    return g;
}
// the plan's lists into the pinned upload at `h`
void put_plan(uint8_t* h, const GraphLayout& g, const msorb::LocalBaPlan& plan) {
    auto put = [&](size_t off, const std::vector<int>& v) { if (!v.empty()) std::memcpy(h + off, v.data(), v.size() * 4); };
    put(g.free_of_kf, plan.free_of_kf); put(g.kf_of_free, plan.kf_of_free); put(g.point_begin, plan.point_begin);
    put(g.kf_begin, plan.kf_begin); put(g.kf_edge, plan.kf_edge); put(g.pair_begin, plan.pair_begin); put(g.pair_i, plan.pair_i);
    put(g.pair_j, plan.pair_j); put(g.pair_a, plan.pair_a); put(g.pair_b, plan.pair_b);
}
// the graph uploaded to `d` becomes A's graph
void wire_graph(BaDev& A, const uint8_t* d, const GraphLayout& g, const msorb::LocalBaPlan& plan, int E) {
    auto ip = [&](size_t off) { return reinterpret_cast<const int*>(d + off); };
    auto fp = [&](size_t off) { return reinterpret_cast<const float*>(d + off); };
    A.Kf = plan.Kf; A.E = E; A.n = 6 * plan.Kf; A.n_pairs = (int)plan.pair_i.size(); A.n_blocks = (E + kEdgeThreads - 1) / kEdgeThreads;
    A.free_of_kf = ip(g.free_of_kf); A.kf_of_free = ip(g.kf_of_free); A.edge_kf = ip(g.edge_kf); A.edge_pt = ip(g.edge_pt);
    A.point_begin = ip(g.point_begin); A.kf_begin = ip(g.kf_begin); A.kf_edge = ip(g.kf_edge); A.pair_begin = ip(g.pair_begin);
    A.pair_i = ip(g.pair_i); A.pair_j = ip(g.pair_j); A.pair_a = ip(g.pair_a); A.pair_b = ip(g.pair_b);
    A.xy = fp(g.xy); A.ur = fp(g.ur); A.w = fp(g.w);
}

// msorb_debug_welding_ba_poll_hook: the calling thread's hook, NULL unless a test set it
struct PollHook { msorb_welding_ba_poll_fn fn = nullptr; void* user = nullptr; };
thread_local PollHook g_poll_hook;

// what one optimize() returns to the engine
struct RunStats {
    int iterations = 0, trials = 0, rejected = 0;
    double chi2_initial = 0, chi2_final = 0, lambda = 0;
    int trial_state = 0;   // the copy of the state at which the last trial's errors were computed: what chi2() reads afterwards
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
    // :1098-1102, :1323-1325 (welding: :3709-3711 alone): nothing touched, the outputs are the inputs
    auto untouched = [&](int status) {
        r->status = status;
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
        if (E && f.welding) std::memset(f.edge_level1, 0, (size_t)E);
        if (f.welding) {
            std::memset(f.wr, 0, sizeof *f.wr);
            f.wr->status = status;
        }
        return MSORB_OK;
    };
    if (f.local && ((Kf == K && !f.welding) || (stop_flag && *stop_flag))) return untouched(Kf == K && !f.welding ? 1 : 2);
    if (int rc = msorb::require_device(device)) return rc;

    // ---- the device block: [uploaded | state and workspaces | results]
    const int n_blocks = (E + kEdgeThreads - 1) / kEdgeThreads;
    const size_t n_out = f.local ? (size_t)E : 0;
    Carve c;
    const size_t o_kf = c.take((size_t)K * sizeof(msorb_ba_keyframe));
    const GraphLayout g1 = carve_graph(c, K, P, E, plan);
    const size_t o_pose0 = c.take((size_t)K * 56), o_pt0 = c.take((size_t)P * 24);
    const size_t in_bytes = c.at;
    const size_t o_pose1 = c.take((size_t)K * 56), o_pt1 = c.take((size_t)P * 24);
    const size_t o_lin = c.take((size_t)kPlanes * E * 8), o_hpp = c.take((size_t)Kf * 27 * 8), o_hll = c.take((size_t)P * 72);
    const size_t o_dinv = c.take((size_t)P * 72), o_S = c.take((size_t)n * n * 8), o_bs = c.take((size_t)n * 8), o_x = c.take((size_t)n * 8);
    const size_t o_ws = c.take(f.one_workgroup_solve ? 0 : ldlt::workspace_doubles(n) * 8);
    const size_t o_pc = c.take((size_t)n_blocks * 8), o_pv = c.take(((size_t)Kf + P) * 8);
    const size_t o_res = c.take(sizeof(BaRes)), o_out = c.take(n_out);
    // welding: the level-1 flags, the chi2 flags that outlive a round, and the second graph's upload (nothing of it is larger than
    // the first graph's: its edges, free KeyFrames and block pairs are subsets), laid out alike on the device and in pinned memory
    const size_t n_lvl = f.welding ? (size_t)E : 0;
    const size_t o_lvl = c.take(n_lvl), o_chi = c.take(n_lvl);
    Carve c2;
    const GraphLayout g2 = f.welding ? carve_graph(c2, K, P, E, plan) : GraphLayout();
    const size_t in2_bytes = c2.at, o_in2 = c.take(in2_bytes);
    const size_t dev_bytes = c.at;
    // pinned: the upload, then [res | pose | points | outlier | level 1 | the second upload] for the read-backs
    Carve hc;
    hc.at = in_bytes;
    const size_t h_res = hc.take(sizeof(BaRes)), h_pose = hc.take((size_t)K * 56), h_pt = hc.take((size_t)P * 24), h_out = hc.take(n_out);
    const size_t h_lvl = hc.take(n_lvl), h_in2 = hc.take(in2_bytes);
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
    put_plan(h, g1, plan);
    put(g1.edge_kf, edge_kf, (size_t)E * 4);
    put(g1.edge_pt, edge_point, (size_t)E * 4);
    put(g1.xy, xy, (size_t)E * 8);
    put(g1.ur, u_right, (size_t)E * 4);
    put(g1.w, inv_sigma2, (size_t)E * 4);
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
    A.K = K; A.P = P;
    A.kf = reinterpret_cast<const msorb_ba_keyframe*>(d + o_kf);
    wire_graph(A, d, g1, plan, E);
    auto dp = [&](size_t off) { return reinterpret_cast<double*>(d + off); };
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
    BA_TRY(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s));
    // the second copy of the state starts equal to the first (a fixed KeyFrame is never written again)
    BA_TRY(hipMemcpyAsync(d + o_pose1, d + o_pose0, (size_t)K * 56, hipMemcpyDeviceToDevice, s));
    if (elapsed_ms) BA_TRY(hipEventRecord(scr.ev[0], s));

    int cur = 0;   // which copy of the state is the estimate; it outlives a run
    std::memset(r, 0, sizeof *r);   // (global's first write of it)
    int round_no = 0;
    // SparseOptimizer::terminate.  where: MSORB_WELDING_POLL_*; the welding entry's test hook sees every poll before the flag is read
    auto stopped = [&](int where, int iteration, int trials) {
        if (f.welding && g_poll_hook.fn) g_poll_hook.fn(g_poll_hook.user, round_no, where, iteration, trials);
        return stop_flag && *stop_flag;
    };
    // ---- SparseOptimizer::optimize(max_iterations) over the graph of A, from the state copy `cur` ----
    auto run = [&](const BaDev& A, const ldlt::Work& W, int max_iterations, RunStats& st) -> int {
        const int n = A.n, Kf = A.Kf, n_blocks = A.n_blocks;
        const int point_blocks = (P + kEdgeThreads - 1) / kEdgeThreads, kf_blocks = (Kf + 3) / 4;
        const int vtx_blocks = (Kf + P + kEdgeThreads - 1) / kEdgeThreads, task_blocks = (A.n_pairs + Kf + 3) / 4;
        if (n) BA_TRY(hipMemsetAsync(d + o_x, 0, (size_t)n * 8, s));   // a failed first solve leaves x as it was: zero
        double lambda = 0, ni = 2;
        int n_bad = 0, iterations = 0, trials = 0, rejected = 0;
        st = RunStats();
        st.trial_state = cur;
        bool ok = A.E > 0;   // without an edge there is nothing to optimise: zero iterations, the estimates as they came
        for (int it = 0; it < max_iterations && !stopped(MSORB_WELDING_POLL_ITERATION, it, trials) && ok; it++) {   // sparse_optimizer.cpp:376
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
                st.chi2_initial = current;
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
                st.trial_state = cur ^ 1;                    // computeActiveErrors ran there, accepted or not
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
            } while (rho < 0 && qmax < 10 && !stopped(MSORB_WELDING_POLL_REJECTED, it, trials));   // :149
            iterations++;
            st.chi2_final = current;
            if (qmax == 10 || rho == 0) { ok = false; continue; }   // :151-155
            if ((ini - current) * 1e3 < ini) n_bad++;               // :157-162
            else n_bad = 0;
            if (n_bad >= 3) ok = false;                             // :164-167
        }
        if (iterations == 0) st.chi2_final = st.chi2_initial;
        st.iterations = iterations; st.trials = trials; st.rejected = rejected; st.lambda = lambda;
        return MSORB_OK;
    };
    RunStats st[2];
    int status = 0, n_level1 = 0, active_kf = 0, active_points = 0;
    bool levelled = false;
    if (!f.welding) {
        if (int rc = run(A, W, f.iterations, st[0])) return rc;
        if (f.local) BA_LAUNCH(ba_classify_kernel, n_blocks, kEdgeThreads, A, cur);
    } else {
        if (n_lvl) BA_TRY(hipMemsetAsync(d + o_chi, 0, n_lvl, s));
        if (int rc = run(A, W, 5, st[0])) return rc;                // :3713-3714
        // the flag rose between the check of :3709 and the first iteration: the reference would classify errors that were never
        // computed; here it is the early return
        if (E > 0 && st[0].iterations == 0) {
            BA_TRY(hipStreamSynchronize(s));   // (the upload reads the pinned block, which the next call fills)
            return untouched(2);
        }
        levelled = !stopped(MSORB_WELDING_POLL_BETWEEN, st[0].iterations, st[0].trials);   // :3718, bDoMore
        round_no = 1;
        if (!levelled) status = 3;
        if (levelled && E > 0) {
            // :3726-3753: chi2() is what the last computeActiveErrors left, isDepthPositive() reads the estimate
            BA_LAUNCH(ba_classify_welding_kernel, n_blocks, kEdgeThreads, A, st[0].trial_state, cur, 1, (const uint8_t*)nullptr, d + o_chi, d + o_lvl);
            BA_TRY(hipMemcpyAsync(h + h_lvl, d + o_lvl, n_lvl, hipMemcpyDeviceToHost, s));
            // a vertex outside the second graph is written by no kernel of it: both copies of the state hold what round 1 left
            BA_TRY(hipMemcpyAsync(d + (cur ? o_pose0 : o_pose1), d + (cur ? o_pose1 : o_pose0), (size_t)K * 56, hipMemcpyDeviceToDevice, s));
            if (P) BA_TRY(hipMemcpyAsync(d + (cur ? o_pt0 : o_pt1), d + (cur ? o_pt1 : o_pt0), (size_t)P * 24, hipMemcpyDeviceToDevice, s));
            BA_TRY(hipStreamSynchronize(s));
            // ---- initializeOptimization(0) (sparse_optimizer.cpp:199-260): the level-0 edges and the vertices they reach ----
            const uint8_t* lv = h + h_lvl;
            uint8_t* const h2 = h + h_in2;
            int *ekf2 = reinterpret_cast<int*>(h2 + g2.edge_kf), *ept2 = reinterpret_cast<int*>(h2 + g2.edge_pt);
            float *xy2 = reinterpret_cast<float*>(h2 + g2.xy), *ur2 = reinterpret_cast<float*>(h2 + g2.ur), *w2 = reinterpret_cast<float*>(h2 + g2.w);
            static thread_local std::vector<int> fixed2;
            static thread_local msorb::LocalBaPlan plan2;
            fixed2.assign((size_t)K, 1);
            int E2 = 0;
            for (int e = 0; e < E; e++) {
                if (lv[e]) { n_level1++; continue; }
                if (!fixed[edge_kf[e]]) fixed2[edge_kf[e]] = 0;
                ekf2[E2] = edge_kf[e]; ept2[E2] = edge_point[e];
                xy2[2 * (size_t)E2] = xy[2 * (size_t)e]; xy2[2 * (size_t)E2 + 1] = xy[2 * (size_t)e + 1];
                ur2[E2] = u_right[e]; w2[E2] = inv_sigma2[e];
                E2++;
            }
            msorb::build_local_ba_plan(K, fixed2.data(), P, E2, ekf2, ept2, plan2);   // (a subsequence of checked edges)
            put_plan(h2, g2, plan2);
            BA_TRY(hipMemcpyAsync(d + o_in2, h2, in2_bytes, hipMemcpyHostToDevice, s));
            BaDev A2 = A;
            wire_graph(A2, d + o_in2, g2, plan2, E2);
            A2.robust = 0;                                          // :3751, setRobustKernel(0) on every edge
            ldlt::Work W2 = W;
            W2.n = A2.n;
            ldlt::carve_workspace(W2, dp(o_ws));
            active_kf = plan2.Kf;
            for (int p = 0; p < P; p++) active_points += plan2.point_begin[(size_t)p + 1] > plan2.point_begin[p];
            if (int rc = run(A2, W2, 10, st[1])) return rc;         // :3758-3759
        }
        // :3769-3803: the same test.  An edge of the second graph has the chi2 of its last trial, if it ran one; every other edge
        // keeps the chi2 flag it had (a level-1 edge: round 1's); the depth is the estimate's
        const bool second = levelled && st[1].iterations > 0;
        BA_LAUNCH(ba_classify_welding_kernel, n_blocks, kEdgeThreads, A, st[second ? 1 : 0].trial_state, cur, second || !levelled ? 1 : 0,
                  levelled ? (const uint8_t*)(d + o_lvl) : (const uint8_t*)nullptr, d + o_chi, d + o_out);
    }
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
    r->status = status;
    r->iterations = st[0].iterations;
    r->trials = st[0].trials;
    r->rejected_trials = st[0].rejected;
    r->n_outliers = n_outliers;
    r->chi2_initial = st[0].chi2_initial;
    r->chi2_final = st[0].chi2_final;
    r->lambda_final = st[0].lambda;
    if (f.welding) {
        for (int e = 0; e < E; e++) f.edge_level1[e] = levelled ? h[h_lvl + e] : 0;
        msorb_welding_ba_result* w = f.wr;
        std::memset(w, 0, sizeof *w);
        w->status = status;
        w->n_level1 = n_level1;
        w->n_outliers = n_outliers;
        w->active_keyframes = active_kf;
        w->active_points = active_points;
        for (int i = 0; i < 2; i++) {
            msorb_welding_ba_round& o = w->round[i];
            o.iterations = st[i].iterations; o.trials = st[i].trials; o.rejected_trials = st[i].rejected;
            o.chi2_initial = st[i].chi2_initial; o.chi2_final = st[i].chi2_final; o.lambda_final = st[i].lambda;
        }
    }
    return MSORB_OK;
}

}  // namespace

extern "C" int msorb_local_ba_capacity(void) { return kLocalCapacity; }
extern "C" int msorb_bundle_adjustment_capacity(void) { return kGlobalCapacity; }
extern "C" int msorb_local_ba_stage_ms(float ms[4]) { return stage_ms(ms); }
extern "C" int msorb_bundle_adjustment_stage_ms(float ms[4]) { return stage_ms(ms); }
extern "C" int msorb_welding_ba_capacity(void) { return kGlobalCapacity; }
extern "C" int msorb_welding_ba_stage_ms(float ms[4]) { return stage_ms(ms); }
extern "C" void msorb_debug_welding_ba_poll_hook(msorb_welding_ba_poll_fn fn, void* user) {
    g_poll_hook.fn = fn;
    g_poll_hook.user = user;
}

extern "C" int msorb_welding_ba(int device, int n_kf, const msorb_ba_keyframe* kfs, int n_points, const float* pos_w, int n_edges,
                                const int* edge_kf, const int* edge_point, const float* xy, const float* u_right, const float* inv_sigma2,
                                const volatile int* stop_flag, float* kf_qt_out, double* kf_qt_d, float* pos_out, double* pos_d,
                                uint8_t* edge_level1, uint8_t* edge_outlier, msorb_welding_ba_result* r, float* elapsed_ms) {
    if (elapsed_ms) *elapsed_ms = 0;
    if (!r || (n_edges > 0 && !edge_level1)) return MSORB_E_ARG;
    // :3607-3608: (float)sqrt(5.99) as the global bundle adjustment has it; the blocked solve and its capacity and memory check
    Entry f{"welding_ba", kGlobalCapacity, (float)std::sqrt(5.99), 1, 5, false, true, edge_outlier, nullptr};
    f.welding = true;
    f.edge_level1 = edge_level1;
    f.wr = r;
    msorb_ba_result one;
    return ba_engine(f, device, n_kf, kfs, n_points, pos_w, n_edges, edge_kf, edge_point, xy, u_right, inv_sigma2, stop_flag, kf_qt_out,
                     kf_qt_d, pos_out, pos_d, &one, elapsed_ms);
}

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
